"""The call plan of a render (csrc/render_plan.h: what render_impl decides before it touches the device) needs no GPU: a
stand-alone probe, tests/plan_probe.cpp, is compiled with the host compiler (address + undefined sanitizers where they link)
and prints the plan of every case it reads.  Checked here: the record / order decision against its Python mirror
(oracle_lib.product_flags, which the counters tests compare the oracle with the product through), the per-kind thresholds, and the
slab arithmetic."""
import itertools
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle_lib as ol  # noqa: E402

HAND_FRAME, HAND_LIST, HAND_BY_CHUNK, HAND_BY_SAMPLE = range(4)
NODE_SWAP_PURE, NODE_SWAP_ANY = 1, 2

OPTS = dict(traversal=1, wavefront=0, qnodes=1, specialise=1, sched=2, slab_log2=28, stack_lds_depth=-1, refill_k=0, init_k=0, leaf_k=0, reps=0,
            skip_unlit=1, shadow_anyhit=1, chunk_shift=0)
FACTS = dict(N=100, Nt=0, grid_ok=1, has_quantised=1, has_wide=0, colors_finite=1, any_trans=0, any_rough=0, gi=0, bounces=4, num_suns=1, num_bulbs=0)
SHAPE = dict(npix=48 * 27, sample_first=0, sample_count=4, spp=4, accumulate=0, num_listed=-1, counters=0, blocks=1024)


def case(**kw):
    c = dict(OPTS, **FACTS, **SHAPE)
    assert not set(kw) - set(c), set(kw) - set(c)
    c.update(kw)
    return c


@pytest.fixture(scope="module")
def probe():
    """Compiles the probe into a private directory; returns plans(list of cases) -> list of dicts."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    with tempfile.TemporaryDirectory(prefix="mirt_plan_") as tmp:      # private: /tmp is shared between users
        exe = os.path.join(tmp, "plan_probe")
        base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(HERE, "plan_probe.cpp"), "-o", exe]
        if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            r = subprocess.run(base, capture_output=True, text=True)      # (a toolchain without the sanitizer runtimes)
            assert r.returncode == 0, r.stderr

        def plans(cases):
            keys = list(OPTS) + list(FACTS) + list(SHAPE)
            text = "".join(" ".join(str(int(c[k])) for k in keys) + "\n" for c in cases)
            r = subprocess.run([exe], input=text, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            out = [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in r.stdout.splitlines()]
            assert len(out) == len(cases)
            return out
        yield plans


def test_the_record_and_order_decision_equals_its_python_mirror(probe):
    """The full cross product, 648 cases.  `records`: which records the build left -- the kind it makes for the scene (quantised for
    a sphere-only scene, wide for one with triangles), both kinds, or none (N <= 1 or bounds_as_shipped), which the mirror knows as
    qnodes = 0.  Order: FLAG_ORDERED_ALL <-> NODE_SWAP_ANY; FLAG_ORDERED <-> NODE_SWAP_PURE, except that the oracle's wide walk
    (oracle.cpp, traverse_wide, dispatched before the flag is looked at) keeps the reference's order whatever FLAG_ORDERED says."""
    grid = list(itertools.product((0, 1, 2), (0, 1), (0, 1, 2), (False, True), (100, 65535, 65536), (0, 1), ("own", "both", "none")))
    assert len(grid) == 648
    cases = []
    for trav, wf, qn, tri, n, gok, rec in grid:
        cases.append(case(traversal=trav, wavefront=wf, qnodes=qn, N=n, Nt=n // 2 if tri else 0, grid_ok=gok,
                          has_quantised=rec == "both" or (rec == "own" and not tri), has_wide=rec == "both" or (rec == "own" and tri)))
    for g, pl in zip(grid, probe(cases)):
        trav, wf, qn, tri, n, gok, rec = g
        f = ol.product_flags(tri, traversal=trav, wavefront=bool(wf), qnodes=qn if rec != "none" else 0, nprims=n, grid_ok=bool(gok))
        quantised, wide = bool(f & ol.FLAG_QNODES) and not f & ol.FLAG_WIDE, bool(f & ol.FLAG_WIDE)
        order = NODE_SWAP_ANY if f & ol.FLAG_ORDERED_ALL else (NODE_SWAP_PURE if f & ol.FLAG_ORDERED and not wide else 0)
        assert (pl["qn"] and pl["notri"], pl["qn"] and not pl["notri"], pl["swap_mask"]) == (quantised, wide, order), (g, pl)
        assert pl["node_bytes"] == (32 if quantised else 64) and pl["reach_check"] == (1 if quantised or wide else 0), (g, pl)


def test_thresholds_by_kind_of_kernel(probe):
    """Pinned from render_impl as it was before the plan was split off."""
    sphere = case()
    wide = case(N=65536, Nt=1000, has_quantised=0, has_wide=1)
    exact = case(N=1700, Nt=1000, has_quantised=0, has_wide=1)
    got = probe([sphere, wide, exact])
    keys = ("refill_k", "init_k", "leaf_k", "reps", "node_bytes")
    assert [tuple(p[k] for k in keys) for p in got] == [(32, 10, 8, 4, 32), (24, 8, 8, 5, 64), (64, 64, 4, 4, 64)]
    assert [(p["qn"], p["notri"]) for p in got] == [(1, 1), (1, 0), (0, 0)]
    stack_lds = got[0]["stack_lds"]
    # an option > 0 overrides each value; init_k is clamped to refill_k
    for base in (sphere, wide, exact):
        p, q, r = probe([dict(base, refill_k=48, init_k=7, leaf_k=3, reps=6), dict(base, refill_k=5, init_k=9), dict(base, refill_k=5)])
        assert (p["refill_k"], p["init_k"], p["leaf_k"], p["reps"]) == (48, 7, 3, 6)
        assert (q["refill_k"], q["init_k"]) == (5, 5) and (r["refill_k"], r["init_k"]) == (5, 5)
    depths = [-1, 0, 1, stack_lds - 1, stack_lds, stack_lds + 1, 1000, -7]
    got = probe([case(stack_lds_depth=d) for d in depths])
    assert [p["lds_depth"] for p in got] == [d if 0 <= d <= stack_lds else stack_lds for d in depths]


def test_specialisation_pending_and_light_switches(probe):
    plain, bulbs, glass, gi, nonfinite, many, off = probe([
        case(), case(num_bulbs=2), case(any_trans=1), case(gi=3, bounces=4), case(colors_finite=0), case(num_suns=20, num_bulbs=13),
        case(specialise=0, skip_unlit=0, shadow_anyhit=0)])
    assert (plain["nobulb"], plain["nopend"], plain["need_pending"], plain["pending_slots"], plain["skip_unlit"], plain["shadow_anyhit"]) == (1, 1, 0, 0, 1, 1)
    assert (bulbs["nobulb"], bulbs["nopend"]) == (0, 1)
    assert (glass["nopend"], glass["need_pending"], glass["pending_slots"]) == (0, 1, 2 * (4 + 0 + 2))
    assert (gi["nopend"], gi["pending_slots"], gi["shading_rng"]) == (0, 2 * (4 + 3 + 2), 1)
    assert (nonfinite["nobulb"], nonfinite["nopend"], nonfinite["skip_unlit"]) == (0, 0, 0)
    assert many["skip_unlit"] == 0 and many["nobulb"] == 0                      # more than 32 lights
    assert (off["nobulb"], off["nopend"], off["skip_unlit"], off["shadow_anyhit"]) == (0, 0, 0, 0)


SLAB_SWEEP = list(itertools.product((1, 2, 63, 64, 65, 1000, 48 * 27, 1 << 16), (1, 3, 4, 16, 100, 4096), (0, 3, 6, 8, 12, 28)))


def test_slabs_tile_the_part(probe):
    """npix = 1, sample_count > 2^slab_log2 and npix that is no multiple of the slab are all in the sweep."""
    got = probe([case(npix=n, sample_count=c, spp=c, slab_log2=lg) for n, c, lg in SLAB_SWEEP])
    for (n, c, lg), p in zip(SLAB_SWEEP, got):
        sp, ns = p["slab_pixels"], p["nslabs"]
        assert 1 <= sp <= n and (ns - 1) * sp < n <= ns * sp, (n, c, lg, p)          # slabs [k sp, min((k + 1) sp, n)) tile [0, n) exactly
        assert p["slab_samples_max"] == sp * c and (sp * c <= 1 << lg or sp == 1), (n, c, lg, p)
        assert sp == n or (sp + 1) * c > 1 << lg, (n, c, lg, p)                       # ... and are as large as the limit allows
        assert p["launch_samples_max"] == p["slab_samples_max"] and p["listed_max"] == 0 and p["total_samples"] == n * c
    assert any(c > 1 << lg for _, c, lg in SLAB_SWEEP) and any(p["nslabs"] > 1 and n % p["slab_pixels"] for (n, _, _), p in zip(SLAB_SWEEP, got))


def test_a_list_bounds_the_launch(probe):
    sweep = [(n, c, lg, listed) for n, c, lg in SLAB_SWEEP[::5] for listed in (1, 100, n)]
    got = probe([case(npix=n, sample_count=c, spp=c, slab_log2=lg, accumulate=1, num_listed=m) for n, c, lg, m in sweep])
    for (n, c, lg, m), p in zip(sweep, got):
        assert p["listed_max"] == min(m, p["slab_pixels"]) and p["launch_samples_max"] == min(m, p["slab_pixels"]) * c, (n, c, lg, m, p)
        assert p["hand_out"] == HAND_LIST


def test_who_hands_the_samples_out(probe):
    """A list always gives list order; sched = 2 falls back to frame order above 3 Gi samples a call and from 2^31 - 1 samples a
    launch; sched = 1 applies only to one-slab, non-wavefront, non-list calls."""
    cases = {
        "by sample": case(), "by sample, slabs": case(slab_log2=8, sample_count=16, spp=16),
        "by chunk": case(sched=1), "by chunk, slabs": case(sched=1, slab_log2=8), "off": case(sched=0),
        "wavefront 1": case(sched=1, wavefront=1), "wavefront 2": case(wavefront=1),
        "list 0": case(sched=0, accumulate=1, num_listed=100), "list 1": case(sched=1, accumulate=1, num_listed=100),
        "list 2": case(sched=2, accumulate=1, num_listed=100, slab_log2=8),
        "3 Gi": case(npix=(3 << 30) // 16, sample_count=16, spp=16), "3 Gi + 16": case(npix=(3 << 30) // 16 + 1, sample_count=16, spp=16),
        "launch 2^31 - 2": case(npix=(1 << 31) - 2, sample_count=1, spp=1, slab_log2=31),
        "launch 2^31 - 1": case(npix=(1 << 31) - 1, sample_count=1, spp=1, slab_log2=31),
    }
    want = {"by sample": HAND_BY_SAMPLE, "by sample, slabs": HAND_BY_SAMPLE, "by chunk": HAND_BY_CHUNK, "by chunk, slabs": HAND_FRAME, "off": HAND_FRAME,
            "wavefront 1": HAND_FRAME, "wavefront 2": HAND_FRAME, "list 0": HAND_LIST, "list 1": HAND_LIST, "list 2": HAND_LIST,
            "3 Gi": HAND_BY_SAMPLE, "3 Gi + 16": HAND_FRAME, "launch 2^31 - 2": HAND_BY_SAMPLE, "launch 2^31 - 1": HAND_FRAME}
    got = dict(zip(cases, probe(list(cases.values()))))
    assert {k: p["hand_out"] for k, p in got.items()} == want
    assert got["by sample, slabs"]["nslabs"] == 81 and got["3 Gi + 16"]["nslabs"] > 1


def test_chunk_size_follows_the_grid(probe):
    """256 samples, smaller while a wave would get fewer than 16 chunks, never below 64; an option >= 4 overrides."""
    blocks = 1024
    ns = [1, 16 * blocks * 64 - 1, 16 * blocks * 64, 16 * blocks * 128 - 1, 16 * blocks * 128, 16 * blocks * 256 - 1, 16 * blocks * 256, 1 << 28]
    got = probe([case(npix=n, sample_count=1, spp=1, blocks=blocks) for n in ns] + [case(chunk_shift=3), case(chunk_shift=4), case(chunk_shift=10)])
    assert [p["chunk_shift"] for p in got] == [6, 6, 6, 6, 7, 7, 8, 8, 6, 4, 10]


def test_the_seed_and_table_choice(probe):
    one, many, acc, acc1 = probe([case(sample_count=1, spp=0), case(sample_count=16, spp=16), case(accumulate=1, sample_first=8, sample_count=4, spp=16),
                                  case(accumulate=1, sample_first=0, sample_count=1, spp=1)])
    assert (one["per_pixel_seed"], one["args_spp"], one["rng_sample_tables"]) == (0, 0, 0)
    assert (many["per_pixel_seed"], many["args_spp"], many["rng_sample_tables"]) == (1, 16, 16)
    assert (acc["per_pixel_seed"], acc["args_spp"], acc["rng_sample_tables"]) == (1, 16, 12)
    assert (acc1["per_pixel_seed"], acc1["args_spp"], acc1["rng_sample_tables"]) == (1, 2, 1)

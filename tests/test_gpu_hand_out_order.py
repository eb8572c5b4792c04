"""What the hand-out orders are made from and what they come out as, read back and compared exactly (tests/sort_ref.py).

  cost_key         (sched = 2: a sample's cost class) through mirt_probe_sched against the restatement, on every step count up to 4096,
                   around every power of two, and at its ends; non-increasing in the step count, never below 255 - 4 31 - 3.
  order_kernel     (sched = 1: the chunk order) through mirt_probe_sched: a permutation, bins non-decreasing, every run of equal bins
                   inside one thread's slice kept together and ascending.  The order between runs of one bin is left open.
  the table        (sched = 2) through mirt_get_sample_order after the measuring frame: the stable argsort of the keys the frame
                   stamped -- most expensive class first, frame order within a class -- per launch; the keys in range and of more
                   than one class; the identity where no sample takes a step; no table before a frame has measured one, and the
                   same table after a geometry update ("The hand-out order is kept").
  the keys         a property of the sample, not of the schedule: equal across fresh scenes and under other reps, leaf_k, refill_k
                   and specialise; and their classes bracket the sum of the frame's step counters, which the kernel counts on its own.
"""
import os

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
import edge_scenes
import sort_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = [("tenthousand", 200, 120, 16), ("redchair", 160, 90, 32)]
u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)      # noqa: E731


# ---- cost_key ----------------------------------------------------------------------------------------------------------------
def test_the_cost_key_is_four_classes_per_doubling():
    around = [v for k in range(32) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1, 5 * (1 << k) // 4 if k >= 2 else 1 << k)]
    steps = np.unique(u32(list(range(4097)) + around + [0xFFFFFFFF]))      # (ascending)
    assert steps[-1] == 0xFFFFFFFF and {(1 << 31) - 1, 1 << 31, (1 << 31) + 1, 5 << 29} <= set(steps.tolist())
    got = api.probe_sched(0, steps)
    assert np.array_equal(got, R.cost_key(steps)), np.flatnonzero(got != R.cost_key(steps))[:5]
    assert (np.diff(got.astype(np.int64)) <= 0).all()
    assert got.min() == R.MIN_KEY and got.max() == 255 and got[0] == 255 and got[-1] == R.MIN_KEY


# ---- order_kernel ------------------------------------------------------------------------------------------------------------
def _cost_sets(n):
    rng = np.random.default_rng([950, n])
    high = rng.integers(0, 8192, n)
    pick = rng.random(n) < 0.3
    high[pick] = rng.choice([8191, 8192, 8193, 20000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], n)[pick]
    return [("all 0", np.zeros(n)), ("all equal", np.full(n, 4000)), ("8 i", 8 * np.arange(n)), ("random below 8192", rng.integers(0, 8192, n)),
            ("some at or above 8192", high), ("all above 8192", np.full(n, 0xFFFFFFFF))]


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 2049, 5000])
def test_the_chunk_order_is_by_bin_and_keeps_every_run(n):
    for name, cost in _cost_sets(n):
        cost = u32(cost)
        order = api.probe_sched(1, cost)
        assert R.chunk_order_faults(cost, order) == [], name
    # the clamp: a cost of 8192 or more sorts with the most expensive bin, before 8191
    cost = u32([0, 8191, 8192, 0xFFFFFFFF, 8184][:n])
    order = api.probe_sched(1, cost)
    assert R.chunk_order_faults(cost, order) == [] and (n < 5 or sorted(order[:4].tolist()) == [1, 2, 3, 4] and order[4] == 0)


def test_bad_arguments_are_errors():
    x, out = np.arange(4, dtype=np.uint32), np.zeros(4, np.uint32)
    for args in ((0, 0, 0, x.ctypes.data, out.ctypes.data), (0, 2, 4, x.ctypes.data, out.ctypes.data), (0, -1, 4, x.ctypes.data, out.ctypes.data),
                 (0, 0, 4, None, out.ctypes.data), (0, 1, 4, x.ctypes.data, None)):
        assert m.lib().mirt_probe_sched(*args) == 3, args
        assert "mirt_probe_sched: bad argument" in m.lib().mirt_last_error().decode()
    assert m.lib().mirt_get_sample_order(None, None, None, None, None) == 3
    assert "mirt_get_sample_order: null scene" in m.lib().mirt_last_error().decode()


# ---- the table ---------------------------------------------------------------------------------------------------------------
def _scene(source, **options):
    """A fresh built scene of a bundled file's name or of a scene text."""
    text = source if "\n" in source else open(os.path.join(ROOT, "scenes", source + ".txt")).read()
    raw = m.initRawConfigFromStl(m.parseText(text), 0)
    for k, v in options.items():
        raw.set_option(k, v)
    m.build_lbvh_karas(raw)
    return raw


def _frame(raw, w, h, spp, counters=False):
    img = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    m.render(img, w, h, spp, raw, params=api.render_params(w, h, spp, counters=counters))
    torch.cuda.synchronize()
    return img.cpu().numpy()


def _no_table(raw):
    with pytest.raises(m.MirtError) as e:
        raw.sample_order()
    assert e.value.status == 6 and "mirt_get_sample_order: the scene has no sample order" in e.value.message


_measured = {}


def _measured_keys(name, w, h, spp):
    """The keys the measuring frame of a fresh default scene stamps: computed once, shared, never written."""
    if (name, w, h, spp) not in _measured:
        raw = _scene(name)
        _frame(raw, w, h, spp)
        keys = raw.sample_order()["keys"]
        raw.close()
        keys.setflags(write=False)
        _measured[(name, w, h, spp)] = keys
    return _measured[(name, w, h, spp)]


@pytest.mark.parametrize("name,w,h,spp", FRAMES)
def test_the_table_of_a_one_launch_frame_is_the_stable_argsort_of_its_keys(name, w, h, spp):
    raw = _scene(name)
    assert raw.get_option("sched") == 2
    _no_table(raw)                                   # before any frame
    _frame(raw, w, h, spp)                           # the measuring frame
    t = raw.sample_order()
    n = w * h * spp
    assert t["total_samples"] == n == t["last_launch_samples"] and len(t["order"]) == n and len(t["keys"]) == n == len(t["sorted_keys"])
    keys = t["keys"]
    assert R.key_is_valid(keys).all(), np.unique(keys[~R.key_is_valid(keys)])
    assert len(np.unique(keys)) > 1                  # (one class alone would prove nothing about the order)
    assert np.array_equal(t["order"], np.argsort(keys, kind="stable"))
    assert np.array_equal(t["sorted_keys"], keys[t["order"]])
    assert np.array_equal(keys, _measured_keys(name, w, h, spp))
    # the ordered frames read the table and leave it alone
    for _ in range(2):
        _frame(raw, w, h, spp)
    again = raw.sample_order()
    assert all(np.array_equal(again[k], t[k]) for k in ("order", "keys", "sorted_keys"))
    raw.close()


@pytest.mark.parametrize("name,w,h,spp", FRAMES)
def test_every_launch_of_a_slabbed_frame_owns_a_permutation_of_its_samples(name, w, h, spp):
    raw = _scene(name, slab_log2=12)
    _frame(raw, w, h, spp)
    t = raw.sample_order()
    n, seg = w * h * spp, (4096 // spp) * spp        # (render_plan.h: 2^slab_log2 / spp pixels a launch)
    launches = -(-n // seg)
    assert raw.stats()["trace_launches"] == launches > 1
    assert t["total_samples"] == n and t["last_launch_samples"] == n - (launches - 1) * seg
    for k in range(launches):
        part = t["order"][k * seg:(k + 1) * seg]
        assert np.array_equal(np.sort(part), np.arange(len(part))), k
    last = t["order"][(launches - 1) * seg:]
    assert R.key_is_valid(t["keys"]).all()
    assert np.array_equal(last, np.argsort(t["keys"], kind="stable")) and np.array_equal(t["sorted_keys"], t["keys"][last])
    # the last launch's samples are the frame's last: the same keys as in the one-launch frame
    assert np.array_equal(t["keys"], _measured_keys(name, w, h, spp)[(launches - 1) * seg:])
    raw.close()


@pytest.mark.parametrize("scene", ["empty", "plane_only"])
def test_a_frame_without_a_traversal_step_has_the_identity(scene):
    raw = _scene(edge_scenes.ALL[scene]())
    w, h, spp = 64, 48, 4
    _frame(raw, w, h, spp)
    t = raw.sample_order()
    assert (t["keys"] == 255).all() and len(t["keys"]) == w * h * spp
    assert np.array_equal(t["order"], np.arange(w * h * spp)) and np.array_equal(t["sorted_keys"], t["keys"])
    raw.close()


def test_no_table_without_a_measurement_and_the_same_table_after_an_update():
    name, w, h, spp = "tenthousand", 96, 54, 8
    off = _scene(name, sched=0)
    _no_table(off)
    _frame(off, w, h, spp)
    _no_table(off)                                   # sched = 0 measures nothing
    off.close()
    chunks = _scene(name, sched=1)
    _frame(chunks, w, h, spp)
    _no_table(chunks)                                # sched = 1 keeps its order per context, by chunk
    chunks.close()

    raw = _scene(name)
    _frame(raw, w, h, spp)
    before = raw.sample_order()
    xyzr = torch.from_numpy(_xyzr(name)).to("cuda")
    xyzr[:, 0] += 0.5
    m.update_spheres(raw, xyzr)
    m.build_lbvh_karas(raw)
    # The table is kept across a geometry update on purpose (a permutation keyed by the frame's shape serves any content): the
    # call answers with the table measured before the update, and frames of that shape go on reading it.
    kept = raw.sample_order()
    assert all(np.array_equal(kept[k], before[k]) for k in ("order", "keys", "sorted_keys")) and kept["total_samples"] == before["total_samples"]
    _frame(raw, w, h, spp)
    kept = raw.sample_order()
    assert all(np.array_equal(kept[k], before[k]) for k in ("order", "keys", "sorted_keys"))
    # another shape measures afresh, on the moved geometry
    _frame(raw, w, h, spp + 8)
    fresh = raw.sample_order()
    assert fresh["total_samples"] == w * h * (spp + 8) and np.array_equal(fresh["order"], np.argsort(fresh["keys"], kind="stable"))
    raw.close()


def _xyzr(name):
    """cx, cy, cz, r of a bundled scene's spheres, file order: float32 [n, 4]."""
    stl = m.parseText(open(os.path.join(ROOT, "scenes", name + ".txt")).read())      # (owns what array() views)
    sph = stl.array("spheres")
    return np.concatenate([sph["c"], sph["r"][:, None]], axis=1).astype(np.float32)


# ---- the keys ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h,spp", FRAMES)
@pytest.mark.parametrize("options", [dict(), dict(reps=1), dict(reps=8), dict(leaf_k=1), dict(leaf_k=64), dict(refill_k=8), dict(specialise=0),
                                     dict(reps=2, leaf_k=16, refill_k=48, specialise=0)], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_the_keys_belong_to_the_sample_not_to_the_schedule(options, name, w, h, spp):
    """render.hip: "each ray still performs exactly the same sequence of steps" whatever the lanes beside it do."""
    want = _measured_keys(name, w, h, spp)
    raw = _scene(name, **options)
    _frame(raw, w, h, spp)
    got = raw.sample_order()["keys"]
    raw.close()
    assert np.array_equal(got, want), (int((got != want).sum()), np.flatnonzero(got != want)[:5])


@pytest.mark.parametrize("name,w,h,spp", FRAMES)
def test_the_classes_bracket_the_steps_the_kernel_counts(name, w, h, spp):
    """An anchor outside cost_key and the sort: every traversal step of the trace kernel adds one to its sample's step count and
    one to exactly one of internal_visits, sphere_tests, tri_tests (render.hip, the step loop), so over a frame the three counters
    add up to the sum of the samples' step counts -- which lies between the sums of the class bounds of the keys stamped."""
    raw = _scene(name, traversal=1, qnodes=0)      # the exact-record walk
    _frame(raw, w, h, spp, counters=True)
    st = raw.stats()
    keys = raw.sample_order()["keys"]
    raw.close()
    steps = st["internal_visits"] + st["sphere_tests"] + st["tri_tests"]
    lo, hi = R.class_bounds(keys)
    assert st["samples"] == w * h * spp == len(keys) and steps > 0
    assert int(lo.sum()) <= steps < int(hi.sum()), (int(lo.sum()), steps, int(hi.sum()))

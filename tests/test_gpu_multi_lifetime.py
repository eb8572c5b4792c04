"""A multi-GPU object that has used every slot gives all of it back when it is closed.

mirt_multi_* with MIRT_MULTI_GATHER=copy and devices [0, 0]: two parts time-sharing GPU 0, the rehearsal of the N > 1 path that a
one-GPU box allows.  Per cycle: create, one frame, MIRT_MULTI_MAX_IN_FLIGHT frames submitted with different stripe_rows and then
waited for (so every slot has allocated its part buffers, `gathered` and `frame`), one frame of twice the size (the part buffers
and the frame of one slot grow once), close.  Every frame equals the single-GPU render of its size byte for byte.  Inside each
counted cycle three creations fail by argument with a status (MirtError): devices [0, 0] without the copy gather ("a device is
listed twice"; on a box with one GPU the count is checked first and the message is "more GPUs requested than present") and a
device index the box does not have ("bad device index"), both refused before mirt_multi_create makes anything; and a scene
description with a negative count, which mirt_scene_create refuses on every device's thread AFTER the object and its vectors
are made, so that the bound also covers the teardown of a half-made object.  A submit beyond MIRT_MULTI_MAX_IN_FLIGHT is
refused with a status too, which ties the test's copy of that constant to the header's.

Free device memory (torch.cuda.mem_get_info) is read as tests/test_gpu_scene_lifetime.py reads it: before an object exists, with
the first counted object used and alive -- the drop is F, what one object holds: two scenes, their streams' workspaces, the slots'
buffers -- and after each close() of nine cycles.  Asserted: F > 0, and free memory after the ninth close() is lower than after
the first by less than F.  So the test sees a leak of F/8 or more per cycle (an object, or one of its two scenes, not given back);
smaller ones are the business of tests/test_dev_mem.py and of review, as for the scene.

Torch's caching allocator is kept out of the readings: the single-GPU references are rendered first, and one uncounted cycle
runs before the first reading."""
import types

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
from conftest import scene_path

pytestmark = pytest.mark.gpu

CYCLES = 9
W, H, SPP = 48, 27, 2
IN_FLIGHT = 4      # MIRT_MULTI_MAX_IN_FLIGHT (include/mirt.h)


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_nine_multi_gpu_objects_leave_no_more_behind_than_one(monkeypatch):
    stl = m.parseInput(scene_path("tri"))
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    want = {}
    for w, h in ((W, H), (2 * W, 2 * H)):
        img = torch.empty(w * h * 4, dtype=torch.uint8, device="cuda")
        m.render(img, w, h, SPP, raw)
        torch.cuda.synchronize()
        want[w] = img.cpu().numpy().reshape(h, w, 4)
        del img
    raw.close()
    monkeypatch.setenv("MIRT_MULTI_GATHER", "copy")

    def use(mg):
        frame, st = mg.render_frame(W, H, SPP)
        assert np.array_equal(frame, want[W]) and st["num_gpus"] == 2
        bufs = [np.zeros((H, W, 4), np.uint8) for _ in range(IN_FLIGHT)]
        tickets = [mg.submit(W, H, SPP, stripe_rows=1 + i, out=b) for i, b in enumerate(bufs)]
        with pytest.raises(m.MirtError, match="frames are in flight"):      # every slot is in use: IN_FLIGHT is the header's value
            mg.submit(W, H, SPP)
        for t, b in zip(tickets, bufs):
            mg.wait(t)
            assert np.array_equal(b, want[W])
        frame, _ = mg.render_frame(2 * W, 2 * H, SPP)
        assert np.array_equal(frame, want[2 * W])
        assert mg.stats(0)["overflow_events"] == 0 and mg.stats(1)["overflow_events"] == 0

    bad = type(stl.desc).from_buffer_copy(stl.desc)      # (the same arrays, which `stl` keeps alive)
    bad.num_spheres = -1
    half = types.SimpleNamespace(desc=bad)

    def refused():
        monkeypatch.delenv("MIRT_MULTI_GATHER")
        with pytest.raises(m.MirtError, match="listed twice|more GPUs requested than present"):
            api.MultiGpu(stl, 2, devices=[0, 0])
        monkeypatch.setenv("MIRT_MULTI_GATHER", "copy")
        with pytest.raises(m.MirtError, match="bad device index"):
            api.MultiGpu(stl, 2, devices=[0, 4096])
        with pytest.raises(m.MirtError, match="negative count"):
            api.MultiGpu(half, 2, devices=[0, 0])

    warm = api.MultiGpu(stl, 2, devices=[0, 0])
    try:
        use(warm)
    finally:
        warm.close()

    before = free_bytes()
    after_close, held = [], None
    for cycle in range(CYCLES):
        mg = api.MultiGpu(stl, 2, devices=[0, 0])
        try:
            use(mg)
            if cycle == 0:
                held = before - free_bytes()      # F
            refused()
        finally:
            mg.close()
        after_close.append(free_bytes())
    lost = after_close[0] - after_close[-1]
    print(f"frames {W}x{H} and {2 * W}x{2 * H}, 2 parts on one GPU: F = {held} B; free before {before} B; after each close, relative to before: "
          f"{[a - before for a in after_close]}; lost over {CYCLES} cycles {lost} B")
    assert held > 0, "a live object must show in the reading, or the test is blind"
    assert lost < held, (lost, held)

"""A scene that has allocated every lazy workspace gives all of it back when it is closed.

The workspaces are filled by the call sequence of test_gpu_call_sequence.py (scene `tri`: the four contexts and their grown
buffers, the pixel-list tables, the wavefront pool, the chunk orders, the by-sample table, the rng tables) plus, per cycle, one
material update (the flag bytes, the reduction's word and its pinned copy), one set_lights (the pinned staging buffer), one
camera_rays and one trace_rays.  Free device memory (torch.cuda.mem_get_info) is read before a scene exists, with one used scene
alive -- the drop is F, what one scene holds -- and after each close() of nine create-use-destroy cycles.

Asserted: free memory after the ninth close() is lower than after the first by less than F.  So the test sees a leak of F/8 or
more per cycle, and no smaller one: the runtime hands memory out in blocks, and a scene that leaks less than a block a cycle moves
the reading only every few cycles.  Smaller leaks are the business of tests/test_dev_mem.py (the owning types give back what they
hold) and of review (every device pointer of a scene is a member of an owning type).

At the sequence's 48x27 the buffers sized by the frame are small, and F (140 MiB on an MI355X) is almost entirely one step of
130 MiB that arrives with the wavefront call (the test prints where the largest step came): by the sizes in the code, that call's
regrown `stack_spill`, 64 words for every thread of the wavefront trace kernel's persistent grid whatever the frame.  So in
practice the bound catches a scene that does not give that buffer back, or one that leaks F/8 (17.5 MiB) a cycle by other means.

Torch's caching allocator is kept out of the readings: the test's own tensors are made first, and one uncounted cycle runs before
the first reading, so that the tensors the sequence's calls make come out of torch's cache from then on."""
import pytest
import torch

from cuda_ray_tracer_amd import api
from gpu_case import options
from test_gpu_call_sequence import SEQUENCE, H, W, build

pytestmark = pytest.mark.gpu

CYCLES = 9


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_nine_scenes_leave_no_more_behind_than_one():
    probe = build("tri")
    ns, nt = probe.desc.num_spheres, probe.desc.num_triangles
    probe.close()
    assert ns + nt > 0
    mats = torch.zeros((ns if ns else nt, 11), dtype=torch.float32, device="cuda")
    rays = torch.zeros((W * H, 8), dtype=torch.float32, device="cuda")
    hits = torch.zeros((W * H, 6), dtype=torch.int32, device="cuda")

    def use(raw, readings=None):
        for _, opts, call in SEQUENCE:
            with options(raw, **opts):
                call(raw)
            if readings is not None:
                readings.append(free_bytes())
        if ns:
            api.get_sphere_materials(raw, mats)
            api.update_sphere_materials(raw, mats)
        else:
            api.get_triangle_materials(raw, mats)
            api.update_triangle_materials(raw, mats)
        raw.set_lights(*raw.lights())
        api.camera_rays(raw, rays, W, H, 1)
        api.trace_rays(raw, rays, hits)
        assert raw.stats()["overflow_events"] == 0

    warm = build("tri")
    try:
        use(warm)
    finally:
        warm.close()

    before = free_bytes()
    after_close = []
    held, during = None, [before]      # (during: the first cycle's reading after the build and after each call, to see the reading's steps)
    for cycle in range(CYCLES):
        raw = build("tri")
        try:
            if cycle == 0:
                during.append(free_bytes())
            use(raw, during if cycle == 0 else None)
            if cycle == 0:
                held = before - free_bytes()      # F
        finally:
            raw.close()
        after_close.append(free_bytes())
    steps = sorted({abs(a - b) for a, b in zip(during, during[1:])} - {0})
    where = ["build"] + [name for name, _, _ in SEQUENCE]
    largest = max(range(len(during) - 1), key=lambda i: during[i] - during[i + 1])
    lost = after_close[0] - after_close[-1]
    print(f"frame {W}x{H}: F = {held} B; free before {before} B; after each close, relative to before: {[a - before for a in after_close]}; "
          f"steps seen while the first scene filled {steps} B, the largest at '{where[largest]}'; lost over {CYCLES} cycles {lost} B")
    assert held > 0, "a live scene must show in the reading, or the test is blind"
    assert lost < held, (lost, held)

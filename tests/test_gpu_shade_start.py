"""One ray start per shade pass (render.hip, ONE_START; shade_common.h, batch_next / advance with START = false): both arms of the
shade loop only set a ray up, and one start_ray serves every lane that got one in the pass.  In the kernels that take the form
(the LDS-only ones over the quantised records) batch_setup writes the reflection ray's set-up for every lane past the last light
and the batch's origin for every lane; the others keep a start in either arm.  Each scene puts lanes at another edge of that, on
either kind of kernel: the frame's bytes are the oracle's, and every counter -- rays_traversed among them -- is the oracle's.

The scenes are those of test_gpu_shade_loop.py (a few dozen primitives), 64 x 48 at 4 spp, one more at 1 spp; the oracle renders
each (scene, spp) once."""
import functools

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
import oracle_lib as ol
import pyscene
import test_gpu_shade_loop as loop
from gpu_case import COUNTER_KEYS, gpu_render, mirror_flags

pytestmark = pytest.mark.gpu

W, H = loop.W, loop.H
LDS_SLOTS, GENERAL_SLOTS = 23, 24      # stack slots of the kernel that starts rays from LDS / of every other one


def two_suns_16_bounces():
    """Sphere-only, two suns, roughness > 0, 16 bounces: the headline's kernel (trace_kernel<.., 31>) by default."""
    return loop._scene(loop._TWO_SUNS + loop._FLOOR + loop._spheres(30, loop._rough_mirror), bounces=16)


def triangle_and_point_light():
    """The exact-record kernels (a start in either arm): triangles among the spheres, a point light after the suns."""
    return loop.triangles().replace("bounces 4\n", "bounces 4\ncolor 6 5 4\nbulb 0.5 2.5 -2\n", 1)


SCENES = {"two_suns_16_bounces": two_suns_16_bounces, "triangle_and_point_light": triangle_and_point_light,
          "glass_gi": loop.glass_gi,                                       # the pending list, single rays next to batches
          "suns_below_the_horizon": loop.suns_below_the_horizon}          # the floor answers shadow rays: a lane takes two passes

# scene, spp, options, (stack_lds_slots, LDS-only stack) of the kernel that renders it
CASES = {"kernel_31": ("two_suns_16_bounces", 4, {}, (LDS_SLOTS, True)),
         "kernel_31_1spp": ("two_suns_16_bounces", 1, {}, (LDS_SLOTS, True)),
         "kernel_15": ("two_suns_16_bounces", 4, dict(ray_start_lds=0), (GENERAL_SLOTS, True)),
         "general_kernel": ("two_suns_16_bounces", 4, dict(specialise=0), None),
         "exact_records": ("triangle_and_point_light", 4, {}, None),
         "pending_list": ("glass_gi", 4, {}, None),
         "two_passes": ("suns_below_the_horizon", 4, {}, (LDS_SLOTS, True))}


@functools.lru_cache(maxsize=None)
def oracle(scene, spp):
    text = SCENES[scene]()
    stl = m.parseText(text)
    o = ol.OracleScene(pyscene.parse_lines(text.split("\n")), bounds_mode=0)
    ref = o.render(W, H, spp, flags=mirror_flags(stl, o), nthreads=8)
    o.close()
    ref["u8"].setflags(write=False)
    return ref


@pytest.mark.parametrize("case", list(CASES))
def test_the_frame_and_the_counters_are_the_oracles(case):
    scene, spp, options, kernel = CASES[case]
    text = SCENES[scene]()
    raw = m.initRawConfigFromStl(m.parseText(text), 0)
    for k, v in options.items():
        raw.set_option(k, v)
    m.build_lbvh_karas(raw)
    gu, _, st = gpu_render(raw, W, H, spp)
    ran = (raw.get_option("stack_lds_slots"), bool(raw.stack_info()["lds_only"]))
    raw.close()
    ref = oracle(scene, spp)
    if kernel is not None:
        assert ran == kernel, ran
    assert st["rays"] > W * H * spp      # (the scene is hit, and shaded)
    differ = int((gu != ref["u8"].reshape(gu.shape)).sum())
    print(case, "bytes that differ from the oracle's:", differ, "of", gu.size)
    assert differ == 0
    for k in COUNTER_KEYS:
        assert st[k] == ref["stats"][k], (k, st[k], ref["stats"][k])
    assert st["rays_traversed"] == ref["stats"]["traversals"], (st["rays_traversed"], ref["stats"]["traversals"])

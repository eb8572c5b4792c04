"""The kernel whose traversal steps read "not traversing" off the current reference (render.hip, CUR_MARK: a lane that is not
traversing holds REF_NONE there, and the lane's flag is brought up to date once per header pass) takes every ray through the same
steps as the kernels that keep the flag: the same bytes and the same counters as the LDS-only kernel with the flag (option
ray_start_lds = 0) and as the general kernel (stack_lds_depth = 24), and the counters of the oracle.

Scenes, each aimed at one way a lane enters or leaves the steps: three hundred spheres under two suns over a plane, four bounces
-- any-hit exits that leave entries on the stack before the header starts the lane's next ray -- and the same with nearest-hit
shadow rays; a sun below the plane, whose shadow rays the plane blocks before any walk, so the lane comes out of its ray start not
traversing; a scene without a tree and one whose root is a leaf (the plan gives these another kernel: the comparison holds all the
same); the comb scenes of test_gpu_stack_depth.py at depth 22 and 23, where the pop that empties a full stack ends the walk; no
bounces at all."""
import numpy as np
import pytest

import cuda_ray_tracer_amd as m
import oracle_lib as ol
import pyscene
import edge_scenes
from gpu_case import COUNTER_KEYS, check_against_oracle, gpu_render, mirror_flags
from test_gpu_stack_depth import comb, tree_depth

pytestmark = pytest.mark.gpu

W, H, SPP = 96, 64, 4
SLOTS, GENERAL_SLOTS = 23, 24      # START_LDS_SLOTS, STACK_LDS (render_plan.h)


def spheres(n, head, seed=5):
    """n spheres in front of the camera, every value a multiple of 2^-6 (the text round-trips them exactly), after `head`."""
    rng = np.random.default_rng(seed)
    c = np.round(rng.uniform(-2.5, 2.5, (n, 3)) * 64) / 64
    c[:, 2] -= 6.0
    r = np.round(rng.uniform(0.08, 0.3, (n, 1)) * 64) / 64
    out = ["png %d %d step.png\n" % (W, H), head]
    for i, s in enumerate(np.concatenate([c, r], axis=1).astype(np.float32)):
        out.append("color %.2f %.2f %.2f\nshininess %.2f\n" % (0.3 + 0.1 * (i % 7), 0.9 - 0.1 * (i % 5), 0.4 + 0.05 * (i % 11), 0.1 * (i % 5)))
        out.append("sphere %.9g %.9g %.9g %.9g\n" % tuple(float(v) for v in s))
    return "".join(out)


TWO_SUNS = "color 1 0.9 0.8\nsun 1 3 2\ncolor 0.5 0.6 0.9\nsun -2 2 1\n"
PLANE = "color 0.5 0.5 0.6\nshininess 0.3\nplane 0 1 0 3\n"
# name -> (scene text, scene options, slots of the default kernel's stack)
SCENES = {
    "two_suns_bounces4": (lambda: spheres(300, "bounces 4\n" + TWO_SUNS + PLANE), {}, SLOTS),
    "two_suns_nearest_hit_shadows": (lambda: spheres(300, "bounces 4\n" + TWO_SUNS + PLANE), {"shadow_anyhit": 0}, SLOTS),
    # (the second sun shines from below the plane y = -3: every shadow ray towards it meets the plane first)
    "sun_below_the_plane": (lambda: spheres(120, "bounces 3\ncolor 1 1 1\nsun 1 3 2\ncolor 0.9 0.7 0.5\nsun 1 -3 2\n" + PLANE), {}, SLOTS),
    "plane_only": (edge_scenes.plane_only, {}, GENERAL_SLOTS),
    "single_sphere": (edge_scenes.single_sphere, {}, GENERAL_SLOTS),
    "comb22": (lambda: comb(22), {}, SLOTS),
    "comb23": (lambda: comb(23), {}, SLOTS),
    "bounces0": (lambda: spheres(120, "bounces 0\n" + TWO_SUNS + PLANE), {}, SLOTS),
}


def render(raw):
    u8, f32, st = gpu_render(raw, W, H, SPP)
    return u8, f32, st, raw.get_option("stack_lds_slots")


def same(a, b, what):
    assert np.array_equal(a[0], b[0]), what
    for k in COUNTER_KEYS:
        assert a[2][k] == b[2][k], (what, k, a[2][k], b[2][k])


@pytest.mark.parametrize("name", list(SCENES))
def test_three_kernels_one_frame(name):
    make, options, slots = SCENES[name]
    text = make()
    stl = m.parseText(text)
    raw = m.initRawConfigFromStl(stl, 0)
    for k, v in options.items():
        raw.set_option(k, v)
    m.build_lbvh_karas(raw)
    new = render(raw)
    raw.set_option("ray_start_lds", 0)
    flagged = render(raw)
    raw.set_option("ray_start_lds", 1)
    raw.set_option("stack_lds_depth", GENERAL_SLOTS)
    general = render(raw)
    lds_only = raw.stack_info()["lds_only"]
    raw.close()
    assert new[3] == slots and flagged[3] == general[3] == GENERAL_SLOTS and not lds_only
    same(new, flagged, "ray_start_lds = 0")
    same(new, general, "stack_lds_depth = 24")
    o = ol.OracleScene(pyscene.parse_lines(text.split("\n")), bounds_mode=0)
    ref = o.render(W, H, SPP, flags=mirror_flags(stl, o, **options), nthreads=8)
    depth = tree_depth(o.nodes(), o.n) if o.n > 1 else 0
    o.close()
    check_against_oracle(new[1], new[0], new[2], ref)      # pixels, and every counter of COUNTER_KEYS -- max_stack among them
    if name.startswith("comb"):
        assert depth == int(name[4:]) and new[2]["max_stack"] == depth
    if name == "two_suns_bounces4":
        assert new[2]["shadow_rays"] > 0 and new[2]["rays"] > new[2]["samples"]

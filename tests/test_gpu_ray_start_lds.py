"""The kernel whose loop header starts rays from LDS (render.hip, SPEC_START_LDS; the plan's choice: test_ray_start_plan.py)
renders what the kernels it stands in for render: the same bytes and the same counters as the LDS-only kernel with the 24-slot
stack (option ray_start_lds = 0) and as the general kernel (stack_lds_depth = 24), and the counters of the oracle.

Scenes: a root that is a leaf, two, three and forty spheres, tenthousand.txt (D = 20), the comb scenes of
test_gpu_stack_depth.py at depth 22 and 23 -- at 23 every one of the 23 slots is used -- and at 24, where the 24-slot kernel
runs; as many suns as the LDS block holds and one more, no plane and no light at all, and a triangle or a point light, which
keep the variant away.  Then geometry moved in place and the option switched off and on: the block is written by every launch
from that launch's own arguments, so nothing can go stale."""
import os

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
import oracle_lib as ol
import pyscene
from gpu_case import COUNTER_KEYS, check_against_oracle, gpu_render, mirror_flags
from test_gpu_stack_depth import comb, tree_depth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 96, 54, 4
SLOTS, GENERAL_SLOTS, SUNS = 23, 24, 10      # START_LDS_SLOTS, STACK_LDS, START_LDS_SUNS (render_plan.h)


def sphere_values(n, seed=7):
    """n spheres in front of the camera, every value a multiple of 2^-6 (the text round-trips them exactly)."""
    rng = np.random.default_rng(seed)
    c = np.round(rng.uniform(-2.0, 2.0, (n, 3)) * 64) / 64
    c[:, 2] -= 5.0
    r = np.round(rng.uniform(0.1, 0.45, (n, 1)) * 64) / 64
    return np.concatenate([c, r], axis=1).astype(np.float32)


def spheres_text(xyzr, suns=1, plane=True, tail=""):
    out = ["png %d %d start.png\nbounces 3\n" % (W, H)]
    for k in range(suns):
        out.append("color %.2f %.2f %.2f\nsun %d %d %d\n" % (1.0 - 0.1 * k, 0.8, 0.6 + 0.05 * k, 1 + k, 3 - (k % 3), 2 - k))
    if plane:
        out.append("color 0.5 0.5 0.6\nshininess 0.2\nplane 0 1 0 2.5\n")
    for i, s in enumerate(xyzr):
        out.append("color %.2f %.2f %.2f\nshininess %.2f\n" % (0.3 + 0.1 * (i % 7), 0.9 - 0.1 * (i % 5), 0.4 + 0.05 * (i % 11), 0.1 * (i % 4)))
        out.append("sphere %.9g %.9g %.9g %.9g\n" % tuple(float(v) for v in s))
    return "".join(out) + tail


def scene_text(name):
    if name == "tenthousand":
        with open(os.path.join(ROOT, "scenes", "tenthousand.txt")) as f:
            return f.read()
    if name.startswith("comb"):
        return comb(int(name[4:]))
    if name.startswith("spheres"):
        return spheres_text(sphere_values(int(name[7:])))
    return {"many_suns": lambda: spheres_text(sphere_values(40), suns=SUNS + 1),
            "max_suns": lambda: spheres_text(sphere_values(40), suns=SUNS),
            "no_plane_no_sun": lambda: spheres_text(sphere_values(40), suns=0, plane=False),
            "triangle": lambda: spheres_text(sphere_values(40), tail="xyz -1 -1 -4\nxyz 1 -1 -4\nxyz 0 1 -4.5\ncolor 0.9 0.9 0.2\ntri 1 2 3\n"),
            "point_light": lambda: spheres_text(sphere_values(40), tail="color 1 0.9 0.8\nbulb 0 3 -2\n")}[name]()


# scene -> slots of the kernel's stack with the options at their defaults
EXPECT = {"spheres1": GENERAL_SLOTS,      # a root that is a leaf: no quantised records at all, the exact-record kernel
          "spheres2": SLOTS, "spheres3": SLOTS, "spheres40": SLOTS, "tenthousand": SLOTS,
          "comb22": SLOTS, "comb23": SLOTS, "comb24": GENERAL_SLOTS,
          "many_suns": GENERAL_SLOTS, "max_suns": SLOTS, "no_plane_no_sun": SLOTS,
          "triangle": GENERAL_SLOTS, "point_light": GENERAL_SLOTS}


def render(raw):
    u8, f32, st = gpu_render(raw, W, H, SPP)
    return u8, f32, st, raw.get_option("stack_lds_slots")


def built(text, **options):
    stl = m.parseText(text)
    raw = m.initRawConfigFromStl(stl, 0)
    for k, v in options.items():
        raw.set_option(k, v)
    m.build_lbvh_karas(raw)
    return stl, raw


def same(a, b, what):
    assert np.array_equal(a[0], b[0]), what
    for k in COUNTER_KEYS:
        assert a[2][k] == b[2][k], (what, k, a[2][k], b[2][k])


@pytest.mark.parametrize("name", list(EXPECT))
def test_three_kernels_one_frame(name):
    text = scene_text(name)
    stl, raw = built(text)
    assert raw.get_option("ray_start_lds") == 1      # (the default)
    on = render(raw)
    assert on[3] == EXPECT[name], on[3]
    raw.set_option("ray_start_lds", 0)
    off = render(raw)
    raw.set_option("ray_start_lds", 1)
    raw.set_option("stack_lds_depth", GENERAL_SLOTS)
    general = render(raw)
    lds_only = raw.stack_info()["lds_only"]
    raw.set_option("stack_lds_depth", -1)
    again = render(raw)
    raw.close()
    assert off[3] == general[3] == GENERAL_SLOTS and not lds_only and again[3] == EXPECT[name]
    same(on, off, "ray_start_lds = 0")
    same(on, general, "stack_lds_depth = 24")
    same(on, again, "options back at their defaults")
    o = ol.OracleScene(pyscene.parse_lines(text.split("\n")), bounds_mode=0)
    ref = o.render(W, H, SPP, flags=mirror_flags(stl, o), nthreads=8)
    depth = tree_depth(o.nodes(), o.n) if o.n > 1 else 0
    o.close()
    check_against_oracle(on[1], on[0], on[2], ref)      # pixels, and every counter of COUNTER_KEYS -- max_stack among them
    if name.startswith("comb"):
        # the walk really fills the stack to D entries: at D = 23 every slot the kernel has is used
        assert depth == int(name[4:]) and on[2]["max_stack"] == ref["stats"]["max_stack"] == depth


@pytest.mark.parametrize("n", [3, 40])
def test_spheres_moved_in_place_give_the_frame_of_a_fresh_scene(n):
    """An update in place and a rebuild, the option off and on again: every launch writes its own block."""
    before, after = sphere_values(n, seed=11), sphere_values(n, seed=12)
    stl, raw = built(spheres_text(before))
    first = render(raw)
    api.update_spheres(raw, torch.from_numpy(after).cuda())
    m.build_lbvh_karas(raw)
    moved = render(raw)
    raw.set_option("ray_start_lds", 0)
    m.build_lbvh_karas(raw)
    moved_off = render(raw)
    raw.set_option("ray_start_lds", 1)
    moved_back = render(raw)
    # and back again, through an update while the option is off
    raw.set_option("ray_start_lds", 0)
    api.update_spheres(raw, torch.from_numpy(before).cuda())
    m.build_lbvh_karas(raw)
    raw.set_option("ray_start_lds", 1)
    back = render(raw)
    raw.close()
    _, fresh_raw = built(spheres_text(after))
    fresh = render(fresh_raw)
    fresh_raw.close()
    assert first[3] == moved[3] == moved_back[3] == back[3] == fresh[3] == SLOTS and moved_off[3] == GENERAL_SLOTS
    assert not np.array_equal(first[0], moved[0])      # (the move is visible)
    same(moved, fresh, "update + rebuild against a fresh scene")
    same(moved_off, fresh, "ray_start_lds = 0 after the update")
    same(moved_back, fresh, "ray_start_lds back to 1")
    same(back, first, "moved back")
